"""Evaluate and test loops on the device: the meters of `PaletteTrainer.evaluate_one_epoch` (palette/utils.py:769-936, eval_step :610-638; the
meters nerf/utils.py:220-330 and palette/utils.py:52-114) and the images of `PaletteTrainer.test` (palette/utils.py:958-1080).

In the reference every step is a `.cpu().numpy()` round trip of fp32 maps (about 23 floats per pixel at num_basis = 4) and the SSIM meter needs
kornia.  The native frame call leaves all these maps as strided columns of one aux row per ray, so here a frame leaves the device as bytes
(`pnr_palette_sheets`, one launch) plus six doubles of running totals (`pnr_frame_metrics`, one launch) read back once at the end.
There is no fallback: without the HIP library every call here raises."""
import ctypes
import os
import struct
import zlib

import torch

from . import _lib
from ._torch_glue import stream_ptr

_WANT = {"mse": _lib.METRIC_MSE, "loss": _lib.METRIC_MSE, "psnr": _lib.METRIC_PSNR, "ssim": _lib.METRIC_SSIM, "sparsity": _lib.METRIC_SPARSITY,
         "tv": _lib.METRIC_TV}
_SLOT = {"frames": 0, "mse": 1, "psnr": 2, "ssim": 3, "sparsity": 4, "tv": 5}
SWATCH = 100   # palette/utils.py:1019


def _rows(t, n, cols, name):
    """A map as [n, cols] fp32 rows with unit column stride (cols == 0: [n]); a strided view -- columns of the frame call's aux_map -- is passed as it is.
    Returns (tensor to keep alive, row stride in floats)."""
    if t.dtype != torch.float32 or not t.is_cuda:
        raise RuntimeError(f"{name} must be a float32 CUDA tensor (there is no CPU fallback)")
    t = t.reshape(n, cols) if cols else t.reshape(n, 1)
    width = max(cols, 1)
    if t.stride(1) != 1 and width > 1 or (n > 1 and t.stride(0) < width):
        t = t.contiguous()
    return t, (t.stride(0) if n > 1 else width)


def frame_sheets(results, H, W, num_basis=None, basis_color=None, gt_weights=None, linear_to_srgb=False, only=None, _pool=False):
    """The uint8 images of one frame (PaletteTrainer.test, palette/utils.py:993-1038, and the save_images block of evaluate_one_epoch, :852-909)
    from a result dict of render(), in ONE launch.  Returns a dict of device uint8 tensors: rgb [H,W,3] and depth [H,W]; for a full PaletteNeRF
    result (gui_mode = False) also view_dep, direct [H,W,3], basis_img, unscaled_basis_img [H, nb W, 3] and basis_acc [H, nb W] (the bases side by
    side); with `gt_weights` [H,W,nb] weights_guide [H, nb W]; with `basis_color` [nb,3] the swatch strip basis_color [100, 100 nb, 3].
    A NeRF result and a gui_mode result give rgb and depth only.  only: the names to make (default: all that the inputs allow).  The images are
    views of ONE device buffer (16-byte aligned each), so a caller that wants them on the host can move them in one copy."""
    H, W = int(H), int(W)
    n = H * W
    image = results["image"]
    dev = image.device
    a = _lib.SheetArgs()
    a.H, a.W, a.linear_to_srgb = H, W, int(bool(linear_to_srgb))
    keep, out = [], {}

    def src(field, stride_field, t, cols, name):
        t, stride = _rows(t, n, cols, name)
        keep.append(t)
        setattr(a, field, t.data_ptr())
        setattr(a, stride_field, stride)

    plan = []   # (field, key, shape): carved from one buffer below

    def dst(field, key, *shape):
        if only is None or key in only:
            plan.append((field, key, shape))

    src("image", "image_stride", image, 3, "image")
    src("depth", "depth_stride", results["depth"], 0, "depth")
    dst("out_rgb", "rgb", H, W, 3)
    dst("out_depth", "depth", H, W)
    full = "basis_acc" in results
    nb = int(num_basis) if num_basis is not None else (int(results["basis_acc"].shape[-1]) if full else 0)
    if full:
        src("view_dep_rgb", "view_dep_stride", results["view_dep_rgb"], 3, "view_dep_rgb")
        src("direct_rgb", "direct_stride", results["direct_rgb"], 3, "direct_rgb")
        src("basis_rgb", "basis_rgb_stride", results["basis_rgb"], 3 * nb, "basis_rgb")
        src("unscaled_basis_rgb", "unscaled_stride", results["unscaled_basis_rgb"], 3 * nb, "unscaled_basis_rgb")
        src("basis_acc", "basis_acc_stride", results["basis_acc"], nb, "basis_acc")
        dst("out_view_dep", "view_dep", H, W, 3)
        dst("out_direct", "direct", H, W, 3)
        dst("out_basis_img", "basis_img", H, nb * W, 3)
        dst("out_unscaled_basis_img", "unscaled_basis_img", H, nb * W, 3)
        dst("out_basis_acc", "basis_acc", H, nb * W)
        if gt_weights is not None:
            src("gt_weights", "gt_weights_stride", gt_weights, nb, "gt_weights")
            dst("out_weights_guide", "weights_guide", H, nb * W)
        if basis_color is not None:
            bc = basis_color.detach().reshape(nb, 3).contiguous()
            if bc.dtype != torch.float32 or not bc.is_cuda:
                raise RuntimeError("basis_color must be a float32 CUDA tensor")
            keep.append(bc)
            a.basis_color = bc.data_ptr()
            dst("out_basis_color", "basis_color", SWATCH, nb * SWATCH, 3)
    a.num_basis = nb if full else 0
    offsets, total = [], 0
    for _, _, shape in plan:
        offsets.append(total)
        size = 1
        for d in shape:
            size *= d
        total += (size + 15) // 16 * 16
    pool = torch.empty(total, dtype=torch.uint8, device=dev)
    for (field, key, shape), off in zip(plan, offsets):
        size = 1
        for d in shape:
            size *= d
        out[key] = pool[off:off + size].view(*shape)
        setattr(a, field, out[key].data_ptr())
    _lib.check(_lib.load().pnr_palette_sheets(ctypes.byref(a), stream_ptr()), "pnr_palette_sheets")
    if _pool:
        return out, pool, [(key, off, shape) for (_, key, shape), off in zip(plan, offsets)]
    return out


class MeterSet:
    """The running totals of all meters on the device (pnr_frame_metrics): `update` is ONE launch per view for every meter in `want` and does not
    synchronise; `totals()` reads the eight doubles back once.  The meter classes below are views of one set (`MeterSet.meters()`), or own a
    private one."""

    def __init__(self, num_basis=None, want=("psnr", "ssim", "sparsity", "tv"), device=None):
        self.num_basis = None if num_basis is None else int(num_basis)
        self.want = 0
        for w in want:
            self.want |= _WANT[w.lower()]
        self.device = device
        self._totals = self._ws = self._host = None
        self._ws_bytes = 0

    def clear(self):
        if self._totals is not None:
            self._totals.zero_()
        self._host = None

    def update(self, preds, truths, basis_acc=None, srgb_to_linear_truth=False, truth_rgb_out=None, frame_out=None):
        """preds [H,W,3] (any row stride), truths [H,W,3 or 4] in [0,1], basis_acc [H,W,nb] or None -- fp32 on the device.  truth_rgb_out: optional
        contiguous [H,W,3] fp32 that receives the ground-truth colour (eval_step's gt_rgb); frame_out: optional double[8] for this view's values."""
        lib = _lib.load()
        H, W = int(preds.shape[-3]), int(preds.shape[-2])
        n = H * W
        dev = preds.device
        if self._totals is None:
            self._totals = torch.zeros(8, dtype=torch.float64, device=dev)
        need = int(lib.pnr_frame_metrics_workspace_bytes(H, W))
        if self._ws is None or self._ws_bytes < need:
            self._ws, self._ws_bytes = torch.zeros(need, dtype=torch.uint8, device=dev), need   # (zero: the ticket; the kernel resets it itself)
        a = _lib.MetricsArgs()
        a.H, a.W = H, W
        p, a.pred_stride = _rows(preds, n, 3, "preds")
        C = int(truths.shape[-1])
        t = truths.reshape(n, C)
        if t.dtype != torch.float32 or not t.is_cuda:
            raise RuntimeError("truths must be a float32 CUDA tensor (there is no CPU fallback)")
        t = t.contiguous()
        a.pred, a.truth, a.truth_channels, a.srgb_to_linear_truth = p.data_ptr(), t.data_ptr(), C, int(bool(srgb_to_linear_truth))
        w = None
        if basis_acc is not None:
            nb = int(basis_acc.shape[-1])
            if self.num_basis is not None and nb != self.num_basis:
                raise RuntimeError(f"basis_acc has {nb} bases, the meters were made for {self.num_basis}")
            w, a.basis_acc_stride = _rows(basis_acc, n, nb, "basis_acc")
            a.basis_acc, a.num_basis = w.data_ptr(), nb
        a.want = self.want
        if truth_rgb_out is not None:
            if not (truth_rgb_out.dtype == torch.float32 and truth_rgb_out.is_cuda and truth_rgb_out.is_contiguous() and truth_rgb_out.numel() == 3 * n):
                raise RuntimeError("truth_rgb_out must be a contiguous [H, W, 3] float32 CUDA tensor")
            a.truth_rgb_out = truth_rgb_out.data_ptr()
        if frame_out is not None:
            if not (frame_out.dtype == torch.float64 and frame_out.is_cuda and frame_out.is_contiguous() and frame_out.numel() >= 8):
                raise RuntimeError("frame_out must be a contiguous float64 CUDA tensor of 8 values")
            a.frame_out = frame_out.data_ptr()
        a.totals, a.workspace, a.workspace_bytes = self._totals.data_ptr(), self._ws.data_ptr(), self._ws_bytes
        _lib.check(lib.pnr_frame_metrics(ctypes.byref(a), stream_ptr()), "pnr_frame_metrics")
        self._host = None

    def totals(self):
        """The eight totals on the host (frames, mse, psnr, ssim, sparsity, tv, 0, 0): one read-back, kept until the next update."""
        if self._host is None:
            self._host = [0.0] * 8 if self._totals is None else self._totals.cpu().tolist()
        return self._host

    def mean(self, what):
        t = self.totals()
        return t[_SLOT[what]] / t[0]

    def meters(self):
        """[PSNRMeter, SSIMMeter(, SparsityMeter, TVMeter)] over this set, by `want`: update the SET once per view, measure() each."""
        out = []
        if self.want & _lib.METRIC_PSNR:
            out.append(PSNRMeter(meter_set=self))
        if self.want & _lib.METRIC_SSIM:
            out.append(SSIMMeter(meter_set=self))
        if self.num_basis is not None and self.want & _lib.METRIC_SPARSITY:
            out.append(SparsityMeter(self.num_basis, meter_set=self))
        if self.num_basis is not None and self.want & _lib.METRIC_TV:
            out.append(TVMeter(self.num_basis, meter_set=self))
        return out


class _Meter:
    """clear / update / measure / report of the reference's meters over a MeterSet (a shared one, or a private one for a meter used alone)."""
    what, label = "", ""

    def __init__(self, num_basis=None, meter_set=None, device=None):
        self.set = meter_set if meter_set is not None else MeterSet(num_basis, want=(self.what,), device=device)
        self.shared = meter_set is not None

    def clear(self):
        self.set.clear()

    def measure(self):
        return self.set.mean(self.what)

    def write(self, writer, global_step, prefix=""):
        writer.add_scalar(os.path.join(prefix, self.label), self.measure(), global_step)

    def report(self):
        return f"{self.label} = {self.measure():.6f}"


class _ImageMeter(_Meter):
    def update(self, preds, truths):
        """preds, truths [B,H,W,3] (or [H,W,3]) device tensors in [0,1]; launches, does not synchronise.  On a shared set, update the set instead
        (one launch for all its meters)."""
        if self.shared:
            raise RuntimeError("this meter is a view of a shared MeterSet: call MeterSet.update once per view")
        preds = preds.reshape(-1, *preds.shape[-3:])
        truths = truths.reshape(-1, *truths.shape[-3:])
        for b in range(preds.shape[0]):
            self.set.update(preds[b], truths[b])


class PSNRMeter(_ImageMeter):
    """nerf/utils.py:220-252"""
    what, label = "psnr", "PSNR"


class SSIMMeter(_ImageMeter):
    """nerf/utils.py:297-330 (kornia's ssim_loss(window_size=11) as documented; see include/pnr.h)"""
    what, label = "ssim", "SSIM"


class _BasisMeter(_Meter):
    basis_metric = True

    def __init__(self, num_basis, meter_set=None, device=None):
        super().__init__(num_basis, meter_set, device)
        self.num_basis = int(num_basis)

    def update(self, omega):
        """omega [B,H,W,nb] (or [H,W,nb]) device tensor; launches, does not synchronise."""
        if self.shared:
            raise RuntimeError("this meter is a view of a shared MeterSet: call MeterSet.update once per view")
        omega = omega.reshape(-1, *omega.shape[-3:])
        for b in range(omega.shape[0]):
            H, W = omega.shape[1], omega.shape[2]
            if getattr(self, "_dummy", None) is None or self._dummy.shape[:2] != (H, W):
                self._dummy = torch.zeros(H, W, 3, dtype=torch.float32, device=omega.device)   # the launch wants an image pair; its meters are not asked for
            self.set.update(self._dummy, self._dummy, omega[b])


class SparsityMeter(_BasisMeter):
    """palette/utils.py:52-81"""
    what, label = "sparsity", "Sparsity"


class TVMeter(_BasisMeter):
    """palette/utils.py:83-114"""
    what, label = "tv", "TV"


def _is_palette(model):
    return hasattr(model, "num_basis")


def _device_poses(model, poses):
    device = next(model.parameters()).device
    return torch.as_tensor(poses, dtype=torch.float32).reshape(-1, 4, 4).to(device), device


def evaluate_path(model, poses, intrinsics, H, W, images, linear=False, want=("psnr", "ssim", "sparsity", "tv"), sheets=False, consume=None,
                  **render_kwargs):
    """The loop of evaluate_one_epoch (palette/utils.py:769-936) without the trainer: for every held-out view, rays on the device, a frame with
    bg_color = 1 and perturb = False through pipeline.render_queue (frame i + 1 is prepared under frame i), then one meter launch (and, with
    `sheets`, one sheet launch; a model with `hist_weights` also gets the weights_guide sheet).  images: [n,H,W,3 or 4] fp32 in [0,1], host or
    device; linear: the scene's colour space is linear (ground truth through srgb_to_linear, the rgb sheet through linear_to_srgb).
    consume(i, results, sheets_or_None) sees every frame.  Returns {"loss", "PSNR", "SSIM", "Sparsity", "TV", "frames"} (by `want`; no palette
    meters for a NeRF model) from ONE read-back at the end.  EMA swaps stay the caller's, as they are for render()."""
    from . import palette_utils, pipeline
    from . import rays as prays
    poses, device = _device_poses(model, poses)
    n = poses.shape[0]
    palette = _is_palette(model)
    nb = int(model.num_basis) if palette else None
    ms = MeterSet(nb, want=tuple(want) + ("mse",))
    kw = dict(render_kwargs, bg_color=1, perturb=False)
    if palette:
        kw["gui_mode"] = False
    guide = sheets and palette and hasattr(model, "hist_weights")

    def rays_of(i):
        return prays.rays_from_indices(poses[i:i + 1], intrinsics, H, W, None)

    def use(i, r):
        truth = torch.as_tensor(images[i], dtype=torch.float32).to(device, non_blocking=True)
        gt_rgb = torch.empty(H, W, 3, dtype=torch.float32, device=device) if guide else None
        ms.update(r["image"].reshape(H, W, 3), truth, r["basis_acc"].reshape(H, W, nb) if palette else None, srgb_to_linear_truth=linear,
                  truth_rgb_out=gt_rgb)
        sh = None
        if sheets:
            gw = palette_utils.get_palette_weight_with_hist(gt_rgb, model.hist_weights).detach() if guide else None
            sh = frame_sheets(r, H, W, nb, model.basis_color if palette else None, gw, linear_to_srgb=linear)
        return consume(i, r, sh) if consume is not None else None

    pipeline.render_queue(model, rays_of, n, consume=use, **kw)
    t = ms.totals()
    frames = t[0]
    out = {"loss": t[1] / frames if frames else float("nan"), "frames": int(frames)}
    for key, name in (("PSNR", "psnr"), ("SSIM", "ssim"), ("Sparsity", "sparsity"), ("TV", "tv")):
        if ms.want & _WANT[name] and (palette or name in ("psnr", "ssim")):
            out[key] = t[_SLOT[name]] / frames if frames else float("nan")
    return out


# {name}_{t:04d}_{suffix}.png of PaletteTrainer.test (palette/utils.py:1035-1045) <- key of frame_sheets
_TEST_FILES = (("rgb", "rgb"), ("depth", "depth"), ("basis_img", "basis_img"), ("basis_acc", "basis_acc"), ("basis_color", "basis_color"),
               ("view_dep_color", "view_dep"))


def write_png(path, array):
    """An 8-bit grey [H,W] or RGB [H,W,3] uint8 array as a PNG file: stdlib only (zlib, struct), filter type 0 on every row."""
    import numpy as np
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("write_png: a non-empty uint8 [H,W] or [H,W,3] array")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + w * (3 if a.ndim == 3 else 1)), np.uint8)   # a filter byte (0 = none) in front of every row
    rows[:, 1:] = a.reshape(h, -1)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)

    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0))
           + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)


def test_path(model, poses, intrinsics, H, W, linear_to_srgb=False, frames_in_flight=1, to_host=True, save_path=None, name="ngp", **render_kwargs):
    """The loop of PaletteTrainer.test (palette/utils.py:958-1080) with write_video = False: for every pose, rays on the device, a frame, ONE sheet
    launch; the images cross PCIe as bytes.  Returns a dict of the per-frame sheets stacked along a new first axis (rgb, depth; for a PaletteNeRF
    model also view_dep, basis_img, basis_acc, basis_color -- the images `test` writes): numpy arrays, or device tensors with to_host = False.
    With save_path, {name}_{t:04d}_{rgb,depth,basis_img,basis_acc,basis_color,view_dep_color}.png are written (rgb and depth for a NeRF model)."""
    from . import pipeline
    from . import rays as prays
    poses, device = _device_poses(model, poses)
    n = poses.shape[0]
    palette = _is_palette(model)
    kw = dict(render_kwargs)
    if palette:
        kw.setdefault("gui_mode", False)
    if save_path is not None:
        os.makedirs(save_path, exist_ok=True)
    fif = pipeline.FramesInFlight(model, max(1, min(int(frames_in_flight), max(n, 1))), device)

    def rays_of(i):
        return prays.rays_from_indices(poses[i:i + 1], intrinsics, H, W, None)

    names = tuple(key for _, key in _TEST_FILES)   # what `test` writes: no direct / unscaled images

    def use(i, r):
        sh, pool, layout = frame_sheets(r, H, W, int(model.num_basis) if palette else None, model.basis_color if palette else None, None,
                                        linear_to_srgb, only=names, _pool=True)
        if not (to_host or save_path is not None):
            return sh
        flat = pool.cpu().numpy()                   # one copy for all images of the frame
        host = {}
        for key, off, shape in layout:
            size = 1
            for d in shape:
                size *= d
            host[key] = flat[off:off + size].reshape(shape)
        if save_path is not None:
            for suffix, key in _TEST_FILES:
                if key in host:
                    write_png(os.path.join(save_path, f"{name}_{i:04d}_{suffix}.png"), host[key])
        return host if to_host else sh

    try:
        frames = fif.render(rays_of, n, consume=use, **kw)
    finally:
        fif.close()
    if not frames:
        return {}
    if to_host:
        import numpy as np
        return {k: np.stack([f[k] for f in frames]) for k in frames[0]}
    return {k: torch.stack([f[k] for f in frames]) for k in frames[0]}
