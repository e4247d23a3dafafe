"""The training side of the reference's data provider and trainer, on the device (csrc/train_batch.hip, `pnr_train_batch` and
`pnr_error_map_update` in include/pnr.h).

`TrainSet` is NeRFDataset's training half (palette/provider.py:356-410, `collate`) with the stack resident on the GPU as fp32, fp16 (what `-O`
= `--preload` + fp16 holds) or uint8 (a quarter of fp32; exact for 8-bit sources).  `TrainSet.batch` also does the head of
PaletteTrainer.train_step (palette/utils.py:450-478): srgb_to_linear, the per-pixel random background, the alpha blend and
`get_palette_weight_with_hist`.  After the index draws and the background draw -- torch RNG calls in the reference's order, so a torch seed
selects the pixels and the background `rays.get_rays` + the reference's expressions select -- a batch is ONE launch; the view is chosen by an
index on the device and nothing is read back.  `train_step` and `train_epoch` are `train_step` / `train_one_epoch` (palette/utils.py:448-608,
684-767; nerf/utils.py:482-600) on top of `model.render` and `train_loss`.

Deviations from the reference, on purpose: with a half stack the reference draws the background and blends in half, here both are fp32 on the
exactly converted half pixels; the error map lives on the device; `rand_pose` (CLIP random poses) and the `lambda_patchsmooth` pair loss
(default 0 in every script) are not built.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, rays
from ._torch_glue import call, ptr, require
from .train_loss import TERM_NAMES, train_loss

ERROR_CELLS = 128 * 128     # the reference's error grid (provider.py: torch.ones([n, 128 * 128]))
_FORMATS = {"fp32": (_lib.IMAGE_FP32, torch.float32), "fp16": (_lib.IMAGE_FP16, torch.float16), "uint8": (_lib.IMAGE_UINT8, torch.uint8)}

TrainBatch = collections.namedtuple("TrainBatch", "rays_o rays_d gt_rgb bg_color gt_weights gt_clip inds inds_coarse index H W")


def _stack(x, name):
    t = torch.from_numpy(x) if isinstance(x, np.ndarray) else x
    if not torch.is_tensor(t) or t.ndim != 4:
        raise ValueError(f"TrainSet: {name} must be a [V,H,W,C] array, got {tuple(getattr(t, 'shape', ()))}")
    return t


def to_storage(images, storage):
    """A [V,H,W,C] stack (uint8, or floating point in [0, 1]) as the dtype `storage` names.  uint8 bytes are kept as they are (the kernel returns
    u / 255, the loader's `astype(float32) / 255`); a float stack becomes round(x * 255) for "uint8" -- exact when it came from 8-bit files."""
    if storage not in _FORMATS:
        raise ValueError(f"TrainSet: storage must be one of {sorted(_FORMATS)}, got {storage!r}")
    dtype = _FORMATS[storage][1]
    if images.dtype == torch.uint8:
        return images if dtype == torch.uint8 else (images.to(torch.float32) / 255).to(dtype)
    if not images.is_floating_point():
        raise ValueError(f"TrainSet: images must be uint8 or floating point, got {images.dtype}")
    if dtype == torch.uint8:
        return (images.to(torch.float32) * 255).round().clamp(0, 255).to(torch.uint8)
    return images.to(dtype)


class TrainSet:
    """TrainSet(images, poses, intrinsics, H, W, num_rays, feat_images=None, error_map=False, patch_size=1, random_size=0, color_space="srgb",
    storage="fp32" | "fp16" | "uint8").  images [V,H,W,3 or 4], poses [V,4,4], intrinsics (fx, fy, cx, cy), feat_images [V,H,W,D]."""

    def __init__(self, images, poses, intrinsics, H, W, num_rays, feat_images=None, error_map=False, patch_size=1, random_size=0,
                 color_space="srgb", storage="fp32", device="cuda"):
        images = _stack(images, "images")
        V, C = images.shape[0], images.shape[3]
        if tuple(images.shape[1:3]) != (H, W):
            raise ValueError(f"TrainSet: images are {tuple(images.shape[1:3])}, H x W is {(H, W)}")
        if C not in (3, 4):
            raise ValueError(f"TrainSet: images must have 3 or 4 channels, got {C}")
        poses = torch.as_tensor(poses)
        if poses.ndim != 3 or tuple(poses.shape) != (V, 4, 4):
            raise ValueError(f"TrainSet: poses must be [{V},4,4], got {tuple(poses.shape)}")
        if len(intrinsics) != 4:
            raise ValueError("TrainSet: intrinsics are (fx, fy, cx, cy)")
        if color_space not in ("srgb", "linear"):
            raise ValueError(f"TrainSet: color_space must be 'srgb' or 'linear', got {color_space!r}")
        num_rays = min(int(num_rays), H * W)
        if num_rays <= 0:
            raise ValueError("TrainSet: num_rays must be positive (a training set draws its pixels)")
        if patch_size > 1 and num_rays % (patch_size * patch_size) != 0:
            raise ValueError(f"TrainSet: patch_size ** 2 = {patch_size * patch_size} must divide num_rays = {num_rays} (nerf/utils.py:81)")
        if patch_size <= 1 and random_size > 0 and num_rays % 2 != 0:
            raise ValueError("TrainSet: random_size pairs need an even num_rays")
        if feat_images is not None:
            feat_images = _stack(feat_images, "feat_images")
            if tuple(feat_images.shape[:3]) != (V, H, W):
                raise ValueError(f"TrainSet: feat_images must be [{V},{H},{W},D], got {tuple(feat_images.shape)}")
            if storage == "fp16" and feat_images.dtype != torch.float16:
                feat_images = feat_images.to(torch.float16)       # provider.py:342-348: the feature stack follows --fp16
            elif feat_images.dtype not in (torch.float16, torch.float32):
                feat_images = feat_images.to(torch.float32)
        self.V, self.H, self.W, self.C, self.num_rays = V, H, W, C, num_rays
        self.intrinsics = tuple(float(v) for v in intrinsics)
        self.patch_size, self.random_size, self.color_space, self.storage = patch_size, random_size, color_space, storage
        self.device = torch.device(device)
        self.images = to_storage(images, storage).to(self.device).contiguous()
        self.feat_images = None if feat_images is None else feat_images.to(self.device).contiguous()
        self.poses = poses.to(torch.float32).to(self.device).contiguous()
        self.error_map = torch.ones(V, ERROR_CELLS, dtype=torch.float32, device=self.device) if error_map else None

    def __len__(self):
        return self.V

    def epoch_order(self, generator=None):
        """A host permutation of the views (the DataLoader's shuffle), uploaded once: slices `order[i:i + B]` are batch indices on the device."""
        return torch.randperm(self.V, generator=generator).to(self.device)

    def _view_index(self, index):
        if torch.is_tensor(index):
            return require(index.reshape(-1).contiguous(), torch.int64, "index")
        idx = [int(index)] if isinstance(index, (int, np.integer)) else [int(i) for i in index]
        if not idx or min(idx) < 0 or max(idx) >= self.V:
            raise IndexError(f"TrainSet: view index {idx} outside [0, {self.V})")
        return torch.tensor(idx, dtype=torch.int64, device=self.device)

    def _draw(self, view_index):
        emap = None if self.error_map is None else self.error_map[view_index]
        return rays.draw_indices(self.H, self.W, self.num_rays, emap, self.patch_size, self.random_size, view_index.shape[0], self.device)

    def _launch(self, view_index, inds, bg=None, hist=None, want=("rays", "gt_rgb")):
        """One pnr_train_batch launch; `want` names the outputs.  Returns a dict of [B,N,.] fp32 tensors."""
        dev, f32 = self.images.device, torch.float32
        B, N = view_index.shape[0], inds.shape[1]
        inds = require(inds.expand(B, N).contiguous(), torch.int64, "inds")
        a = _lib.TrainBatchArgs()
        a.V, a.H, a.W, a.C, a.B, a.N = self.V, self.H, self.W, self.C, B, N
        a.images, a.image_format = ptr(require(self.images, _FORMATS[self.storage][1], "images")), _FORMATS[self.storage][0]
        a.poses = ptr(self.poses)
        a.fx, a.fy, a.cx, a.cy = self.intrinsics
        a.view_index, a.inds = ptr(view_index), ptr(inds)
        a.srgb_to_linear = int(self.color_space == "linear")
        keep = [inds]
        a.bg_mode, a.bg_const = 0, 1.0
        if torch.is_tensor(bg):
            bg = require(bg.detach().to(dev, f32).contiguous(), f32, "bg_color")
            if bg.numel() == 3:
                a.bg_mode = 1
            elif bg.numel() == 3 * B * N:
                a.bg_mode = 2
            else:
                raise RuntimeError(f"TrainSet: bg_color must be a number, [3] or [B*N,3]; got {tuple(bg.shape)}")
            a.bg_color = ptr(bg)
            keep.append(bg)
        elif bg is not None:
            a.bg_const = float(bg)
        out = {}

        def new(name, width):
            out[name] = torch.empty(B, N, width, dtype=f32, device=dev)
            return ptr(out[name])
        if "rays" in want:
            a.rays_o, a.rays_d = new("rays_o", 3), new("rays_d", 3)
        if "pixels" in want:
            a.pixels = new("pixels", self.C)
        if "gt_rgb" in want:
            a.gt_rgb = new("gt_rgb", 3)
        if hist is not None:
            if hist.ndim == 5 and hist.shape[0] == 1:
                hist = hist[0]
            if hist.ndim != 4:
                raise RuntimeError(f"TrainSet: hist_weights must be [1,nb,R,G,B], got {tuple(hist.shape)}")
            hist = hist.detach()
            if hist.dtype != f32 or not hist.is_cuda:
                raise RuntimeError("hist_weights must be a torch.float32 CUDA tensor")
            keep.append(hist)
            a.hist_weights = ptr(hist)
            a.num_basis, a.Sr, a.Sg, a.Sb = hist.shape
            a.hist_stride = (ctypes.c_uint64 * 4)(*hist.stride())       # the reference's table is a permuted view: read where it lies, no copy per step
            a.gt_weights = new("gt_weights", hist.shape[0])
        if self.feat_images is not None and "gt_clip" in want:
            a.feat_images = ptr(self.feat_images)
            a.feat_format = _lib.IMAGE_FP16 if self.feat_images.dtype == torch.float16 else _lib.IMAGE_FP32
            a.D = self.feat_images.shape[3]
            a.gt_clip = new("gt_clip", a.D)
        call("pnr_train_batch", ctypes.byref(a))
        return out

    def collate(self, index):
        """provider.py:356-410 for a training set: {'H', 'W', 'rays_o', 'rays_d', 'inds', 'images'[, 'feat_images'][, 'index', 'inds_coarse']},
        for a caller who keeps the reference's train_step.  `images` [B,N,C] and `feat_images` [B,N,D] are fp32 (the exactly converted stack)."""
        view_index = self._view_index(index)
        inds, coarse = self._draw(view_index)
        o = self._launch(view_index, inds, want=("rays", "pixels", "gt_clip"))
        res = {"H": self.H, "W": self.W, "rays_o": o["rays_o"], "rays_d": o["rays_d"], "inds": inds, "images": o["pixels"]}
        if "gt_clip" in o:
            res["feat_images"] = o["gt_clip"]
        if coarse is not None:
            res["index"] = view_index
            res["inds_coarse"] = coarse
        return res

    def batch(self, index, model=None, bg_color=None):
        """collate + the head of train_step (palette/utils.py:450-478) -> TrainBatch.  The background follows train_step's rule unless bg_color is
        given: 1 when the images have no alpha or the model has a background model (bg_radius > 0), else a per-pixel torch.rand [B,N,3] (the
        reference's rand_like draw, made after the index draws).  gt_weights only when the model has `hist_weights`."""
        view_index = self._view_index(index)
        inds, coarse = self._draw(view_index)
        B, N = view_index.shape[0], inds.shape[1]
        if bg_color is None:
            if self.C == 3 or (model is not None and getattr(model, "bg_radius", 0) > 0):
                bg_color = 1
            else:
                bg_color = torch.rand(B, N, 3, dtype=torch.float32, device=self.images.device)
        hist = getattr(model, "hist_weights", None) if model is not None else None
        o = self._launch(view_index, inds, bg=bg_color, hist=hist, want=("rays", "gt_rgb", "gt_clip"))
        return TrainBatch(o["rays_o"], o["rays_d"], o["gt_rgb"], bg_color, o.get("gt_weights"), o.get("gt_clip"), inds, coarse, view_index, self.H, self.W)

    def update_error_map(self, batch, loss_ray):
        """palette/utils.py:578-599 on the device-resident map: one launch, no synchronisation.  loss_ray [B,N]: train_loss' info['loss_ray'], the
        per-ray colour error (the reference's `loss` at that point also carries the scalar regularisers, the same number added to every ray)."""
        if self.error_map is None or batch.inds_coarse is None:
            return
        B, N = batch.inds_coarse.shape
        loss_ray = require(loss_ray.detach().reshape(B, N).to(torch.float32).contiguous(), torch.float32, "loss_ray")
        coarse = require(batch.inds_coarse.contiguous(), torch.int64, "inds_coarse")
        call("pnr_error_map_update", ptr(self.error_map), ERROR_CELLS, ptr(batch.index), ptr(coarse), ptr(loss_ray), B, N)


def train_step(model, batch, render_kwargs=None, lambda_sparsity=0.0, lambda_offsets=0.0, lambda_view_dep=0.0, lambda_smooth=0.0, lambda_weight=0.0,
               lambda_palette=0.0, lambda_sparse=0.0, want_outputs=True, lambda_distort=0.0):
    """PaletteTrainer.train_step (palette/utils.py:481-608) / Trainer.train_step (nerf/utils.py:527-536) from the render on, on a TrainBatch:
    returns (pred_rgb, gt_rgb, loss, loss_dict) with loss_dict keyed by train_loss.TERM_NAMES (device scalars; 'loss_ray' [B,N] rides along for
    the error map).  A PaletteNeRF model renders with force_all_rays=True and gets the weight guide, the clip target and the palette anchor; a
    NeRF model renders with force_all_rays=False and rays_gt=gt_rgb, its rgb_norm term weighted by lambda_sparse.  render_kwargs: dt_gamma,
    max_steps, ... as the reference passes **vars(opt).  lambda_weight and lambda_palette are the trainer's per-epoch values (:651-669).
    lambda_distort != 0 renders with distortion=True and adds the distortion loss (train_loss); with 0 the render is not told of it."""
    kw = dict(render_kwargs or {})
    if lambda_distort != 0:
        kw["distortion"] = True
    bg = batch.bg_color.reshape(-1, 3) if torch.is_tensor(batch.bg_color) and batch.bg_color.numel() > 3 else batch.bg_color
    palette = hasattr(model, "num_basis")
    if palette:
        out = model.render(batch.rays_o, batch.rays_d, staged=False, bg_color=bg, perturb=True, force_all_rays=True, **kw)
        origin = getattr(model, "basis_color_origin", None)
        smooth = lambda_smooth if getattr(model, "require_smooth_loss", False) else 0.0        # palette/utils.py:537-541
        loss, info = train_loss(out, batch.gt_rgb, lambda_sparsity=lambda_sparsity, lambda_offsets=lambda_offsets, lambda_view_dep=lambda_view_dep,
                                lambda_smooth=smooth, lambda_weight=lambda_weight, lambda_palette=lambda_palette if origin is not None else 0.0,
                                gt_weights=batch.gt_weights, gt_clip=batch.gt_clip if getattr(model.opt, "pred_clip", False) else None,
                                basis_color=model.basis_color if origin is not None else None, basis_color_origin=origin, want_outputs=want_outputs,
                                lambda_distort=lambda_distort)
    else:
        out = model.render(batch.rays_o, batch.rays_d, rays_gt=batch.gt_rgb, staged=False, bg_color=bg, perturb=True, force_all_rays=False, **kw)
        loss, info = train_loss(out, batch.gt_rgb, lambda_sparse=lambda_sparse, want_outputs=want_outputs, lambda_distort=lambda_distort)
    loss_dict = {name: info["terms"][i] for i, name in enumerate(TERM_NAMES)}
    for extra in ("loss_sparse", "loss_distort"):
        if extra in info:
            loss_dict[extra] = info[extra]
    loss_dict["loss_ray"] = info["loss_ray"]
    return info["image"], batch.gt_rgb, loss, loss_dict


def train_epoch(model, trainset, optimizer, scheduler=None, scaler=None, update_extra_interval=16, global_step=0, batch_size=1, fp16=False,
                render_kwargs=None, generator=None, max_steps=None, ema=None, lambda_distort=0.0, **lambdas):
    """train_one_epoch (palette/utils.py:684-767): one pass over the views in a shuffled order -- update_extra_state every update_extra_interval
    global steps, zero_grad, train_step, backward, optimiser step, the per-step scheduler, the error-map update.  The running loss is summed on the
    device and read back ONCE at the end (the reference's loss.item() per step is a synchronisation).  Returns (average loss, new global_step).
    The per-epoch rules -- the lambda_weight decay, the lambda_palette switch, the smooth-loss switch (:649-674) -- stay the caller's: pass the
    epoch's numbers in **lambdas (train_step's keywords).  lambda_distort != 0 adds the distortion loss (the render is then asked for it:
    distortion=True).  `ema` (an optim.ExponentialMovingAverage or torch_ema's) gets its update() where the reference calls it: ONCE, after the
    pass (palette/utils.py:746-747, nerf/utils.py:920-921; train_gui: after its 16 steps, :789-790) -- not per step."""
    model.train()
    order = trainset.epoch_order(generator)
    total = torch.zeros((), dtype=torch.float32, device=trainset.images.device)
    steps = 0
    for head in range(0, trainset.V - batch_size + 1, batch_size):
        if max_steps is not None and steps >= max_steps:
            break
        # (a PaletteNeRF model has no update_extra_state: its geometry is frozen, and palette/utils.py:706-709 has the call commented out)
        if getattr(model, "cuda_ray", False) and hasattr(model, "update_extra_state") and update_extra_interval and global_step % update_extra_interval == 0:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=fp16):
                model.update_extra_state()
        global_step += 1
        steps += 1
        optimizer.zero_grad(set_to_none=True)
        batch = trainset.batch(order[head:head + batch_size], model)
        with torch.autocast("cuda", dtype=torch.float16, enabled=fp16):
            _, _, loss, loss_dict = train_step(model, batch, render_kwargs, want_outputs=False, lambda_distort=lambda_distort, **lambdas)
        if scaler is not None:
            scaler.scale(loss).backward()
            scaler.step(optimizer)
            scaler.update()
        else:
            loss.backward()
            optimizer.step()
        if scheduler is not None:
            scheduler.step()
        trainset.update_error_map(batch, loss_dict["loss_ray"])
        total += loss.detach()
    if ema is not None:
        ema.update()
    return (float(total) / max(1, steps)), global_step
